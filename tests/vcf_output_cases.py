"""Hand-built record sets for the VCF formatters (secedo_variant_format_host / secedo_variant_format_device) and a
plain Python statement of the text they owe, shared by tests/test_vcf_output_cpu.py and tests/test_gpu_vcf_output.py.
Genotype codes: maternal << 3 | paternal, bases 0..3 = ACGT, 5 = N."""
import numpy as np

from secedo_amd.variant import RECORD_DTYPE

POOLED, COMMON, CLUSTER = 0, 1, 2
INFO = "\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t"
BASES = "ACGTNN"


def g(a, b):
    return a << 3 | b


def chromosome_name(c):
    return str(c + 1) if c < 22 else "X" if c == 22 else "Y"


def lines_of(kind, genotype, ref, chrom, pos, counts):
    """The lines one record yields (variant_calling.cpp:247-321, :395-406), as str."""
    tail = "\t" + "".join("%d " % c for c in counts) + "\n"

    def line(r, alt, gt="1/1"):
        return "%s\t%d\t.\t%s\t%s%s%s%s" % (chrom, pos, r, alt, INFO, gt, tail)
    if kind == POOLED:
        new = genotype & 7
        return [line(BASES[(ref >> 3) & 7 if (ref & 7) == new else ref & 7], BASES[new])]
    if (ref & 7) == (ref >> 3):
        if (genotype & 7) == (genotype >> 3):
            return [line(BASES[ref & 7], BASES[genotype & 7])]
        return [line(BASES[ref & 7], BASES[genotype & 7] + BASES[genotype >> 3], "0/1")]
    r1, r2 = sorted((BASES[ref & 7], BASES[ref >> 3]))
    g1, g2 = sorted((BASES[genotype & 7], BASES[genotype >> 3]))
    if (g1, g2) == (r1, r2):
        return []
    if g1 == r1:
        return [line(r2, g2)]
    if g2 == r2:
        return [line(r1, g1)]
    return [line(r1, g1), line(r2, g2)]


class Case:
    """records: [(locus, kind, cluster, genotype, counts)] in write order."""

    def __init__(self, chr_locus_off, locus_pos, locus_ref, num_clusters, records, preambles=None):
        self.chr_locus_off = np.asarray(chr_locus_off, dtype=np.uint32)
        self.locus_pos = np.asarray(locus_pos, dtype=np.uint32)
        self.locus_ref = np.asarray(locus_ref, dtype=np.uint8)
        self.num_clusters = num_clusters
        self.preambles = preambles
        self.records = np.zeros(len(records), dtype=RECORD_DTYPE)
        for k, (locus, kind, cluster, genotype, counts) in enumerate(records):
            self.records[k] = (locus, cluster, genotype, kind, counts)

    def args(self):
        return (self.records, self.chr_locus_off, self.locus_pos, self.locus_ref, self.num_clusters, self.preambles)

    def expected(self):
        """[cluster_0, ..., common] as bytes."""
        files = [[p.decode()] for p in (self.preambles or [b""] * self.num_clusters)] + [[]]
        for r in self.records:
            locus = int(r["locus"])
            chrom = 0
            while chrom + 1 < len(self.chr_locus_off) - 1 and locus >= self.chr_locus_off[chrom + 1]:
                chrom += 1
            dest = int(r["cluster"]) if r["kind"] == CLUSTER else self.num_clusters
            files[dest] += lines_of(int(r["kind"]), int(r["genotype"]), int(self.locus_ref[locus]),
                                    chromosome_name(chrom), int(self.locus_pos[locus]), [int(c) for c in r["counts"]])
        return ["".join(f).encode() for f in files]


def preambles(n):
    return [("##fileformat=VCFv4.2\n##cluster=%d\n#CHROM\tPOS\tcluster-%d\n" % (i, i)).encode() for i in range(n)]


def digits():
    """Positions and counts at every digit count, in the common file and in a cluster file."""
    pos = [1, 9, 10, 999999999, 4294967295]
    counts = [(0, 9, 10, 65535), (65535, 0, 9, 10), (10, 65535, 0, 9), (9, 10, 65535, 0), (0, 0, 0, 0)]
    recs = []
    for l in range(5):
        recs.append((l, COMMON, 0, g(1, 1), counts[l]))
        recs.append((l, CLUSTER, 1, g(2, 2), counts[(l + 1) % 5]))
    return Case([0, 5], pos, [g(0, 0)] * 5, 2, recs, preambles(2))


def chromosomes():
    """Records in chromosome slots 0, 9, 21, 22, 23 (1, 10, 22, X, Y), the slots between empty; two records of one
    file straddle each change."""
    slots = [0, 9, 21, 22, 23]
    off, n = [0], 0
    for c in range(24):
        n += 2 if c in slots else 0
        off.append(n)
    recs = [(l, kind, 0, g(3, 3), (l, 1, 2, 3)) for l in range(10) for kind in (COMMON, CLUSTER)]
    return Case(off, [100 + l for l in range(10)], [g(0, 0)] * 10, 1, recs, preambles(1))


def line_rules():
    """Homozygous and heterozygous reference with 0, 1 and 2 lines, the two-letter ALT, the pooled ref_base rule."""
    het = g(0, 1)  # A / C
    table = [
        (g(0, 0), COMMON, g(2, 2)),    # homozygous both: 1/1
        (g(0, 0), COMMON, g(2, 3)),    # two-letter ALT, 0/1
        (g(0, 0), COMMON, g(3, 2)),    # the same, other order
        (het, COMMON, g(1, 0)),        # the reference's pair in the other order: no line
        (het, COMMON, g(0, 2)),        # shares the first: one line, C -> G
        (g(0, 3), COMMON, g(1, 3)),    # A/T against C/T: shares the second, one line, A -> C
        (het, COMMON, g(2, 3)),        # shares none: two lines
        (g(1, 0), COMMON, g(3, 2)),    # unsorted reference and genotype: two lines, sorted
        (g(1, 0), POOLED, g(0, 0)),    # new base equals ref & 7, the base looked at first: REF is the other one
        (g(0, 1), POOLED, g(0, 0)),    # equals the other one: REF is ref & 7
        (g(2, 2), POOLED, g(3, 3)),    # equals neither
        (g(5, 5), COMMON, g(1, 1)),    # N in the reference
    ]
    recs, ref = [], []
    for l, (r, kind, geno) in enumerate(table):
        ref.append(r)
        recs.append((l, kind, 0, geno, (l, 2 * l, 30, 4)))
        if kind == COMMON:
            recs.append((l, CLUSTER, l % 3, geno, (7, l, 0, 12345)))
    return Case([0, len(table)], [5 * l + 1 for l in range(len(table))], ref, 3, recs, preambles(3))


def many_clusters(n=300):
    """n cluster files, cluster 7 and the last without a record (preamble only), interleaved destinations."""
    rng = np.random.default_rng(2)
    n_loci = 40
    recs = []
    for l in range(n_loci):
        recs.append((l, POOLED, 0, g(1, 1), (1, 2, 3, 4)))
        for c in sorted(rng.choice(n - 1, 12, replace=False).tolist()):
            if c != 7:
                recs.append((l, CLUSTER, c, g(int(rng.integers(4)), int(rng.integers(4))), tuple(rng.integers(0, 70000, 4) % 65536)))
    ref = [g(int(a), int(b)) for a, b in rng.integers(0, 4, (n_loci, 2))]
    return Case([0, 25, n_loci], np.cumsum(rng.integers(1, 10**6, n_loci)), ref, n, recs, preambles(n))


def long_file(n_loci=2500):
    """One cluster and common, each longer than two BGZF blocks; no line of cluster_0 ends at byte 65280 or 130560."""
    rng = np.random.default_rng(3)
    recs = []
    for l in range(n_loci):
        recs.append((l, COMMON, 0, g(int(rng.integers(4)), int(rng.integers(4))), tuple(rng.integers(0, 300, 4))))
        recs.append((l, CLUSTER, 0, g(int(rng.integers(4)), int(rng.integers(4))), tuple(rng.integers(0, 300, 4))))
    ref = [g(int(a), int(b)) for a, b in rng.integers(0, 4, (n_loci, 2))]
    return Case([0, 1000, n_loci], np.cumsum(rng.integers(1, 5000, n_loci)), ref, 1, recs, preambles(1))


def no_records():
    return Case([0, 0], [], [], 2, [], preambles(2))


ALL = dict(digits=digits, chromosomes=chromosomes, line_rules=line_rules, one_cluster=lambda: long_file(40),
           many_clusters=many_clusters, long_file=long_file, no_records=no_records)
