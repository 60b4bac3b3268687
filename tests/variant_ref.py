"""Plain Python restatement of the reference's variant_calling() (variant_calling.cpp:1-461), the parity
yardstick of the GPU variant calling (as tests/kmeans_ref.py is for the clustering). Written for clarity, not
speed: one locus at a time, the reference's own loops, its u16 count arrays and its tie rules.

`write_files` writes what the reference writes; `##fileDate` is the only line that depends on the time of the
run (compare files with `strip_date`).
"""
import math
import os
import time

NO_GENOTYPE = 255
INT_TO_CHAR = "ACGTNN"
INFO_FORMAT = "\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t"


def char_to_int(c):
    return {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3, "U": 3, "u": 3}.get(c, 5)


def id_to_chromosome(i):
    return str(i + 1) if i < 22 else ("X" if i == 22 else "Y")


def argsort4(n):
    """argsort of util.hpp (std::sort of 4 indices: libstdc++'s insertion sort, stable ascending)."""
    return sorted(range(4), key=lambda j: n[j])  # Python's sort is stable


def likely_homozygous(n_bases, theta):
    cov = sum(n_bases) & 0xFFFF
    if cov < 9:
        return NO_GENOTYPE
    b = max(range(4), key=lambda j: (n_bases[j], -j))  # std::max_element: the first maximum
    if float((cov - n_bases[b]) & 0xFFFFFFFF) <= round_half_away(cov * theta + math.sqrt(cov * theta * (1 - theta))):
        return b + (b << 3)
    return NO_GENOTYPE


def round_half_away(x):
    """std::round of a non-negative x (halves away from zero); NaN stays NaN"""
    if x != x:
        return x
    f = math.floor(x)
    return float(f + 1 if x - f >= 0.5 else f)


def most_likely_genotype(n_bases, likely_homozygous_total, hetero_prior, theta):
    """-> (genotype, u16 coverage)"""
    cov = sum(n_bases) & 0xFFFF
    log_theta = math.log(theta / 3)
    log_one_minus = math.log(1 - theta)
    log_half_minus = math.log(0.5 - theta / 3)
    idx = argsort4(n_bases)
    n = n_bases
    if cov < 9:
        if n[idx[3]] >= ((cov - 1) & 0xFFFFFFFF) and likely_homozygous_total:
            return (idx[3] << 3) | idx[3], cov
        return NO_GENOTYPE, cov
    log_homo = n[idx[3]] * log_one_minus + float((cov - n[idx[3]]) & 0xFFFFFFFF) * log_theta
    log_hetero = (n[idx[2]] + n[idx[3]]) * log_half_minus + (n[idx[0]] + n[idx[1]]) * log_theta + math.log(hetero_prior)
    if log_homo == log_hetero:
        return NO_GENOTYPE, cov
    if log_homo > log_hetero:
        if n[idx[2]] == n[idx[3]]:
            return NO_GENOTYPE, cov
        return (idx[3] << 3) | idx[3], cov
    if n[idx[2]] == n[idx[1]]:
        return NO_GENOTYPE, cov
    std_dev = math.sqrt(0.25 * (n[idx[3]] + n[idx[2]]))
    mean = float((n[idx[3]] + n[idx[2]]) // 2)
    if cov > 15 and abs(n[idx[3]] - mean) <= std_dev and abs(n[idx[2]] - mean) < std_dev:
        return (idx[3] << 3) | idx[2], cov
    return NO_GENOTYPE, cov


# --- the reference genome -----------------------------------------------------------------------------------------

class Stream:
    """The std::ifstream calls get_next_chromosome makes, over the file's bytes."""

    def __init__(self, data):
        self.d, self.pos, self.fail = data, 0, False

    def getline(self):
        if self.fail or self.pos >= len(self.d):
            self.fail = True
            return None
        e = self.d.find(b"\n", self.pos)
        e = len(self.d) if e < 0 else e
        line = self.d[self.pos:e]
        self.pos = e + 1 if e < len(self.d) else len(self.d)
        return line.decode("latin-1")

    def peek(self):
        return None if self.fail or self.pos >= len(self.d) else chr(self.d[self.pos])

    def get(self):
        if self.fail or self.pos >= len(self.d):
            self.fail = True
            return None
        self.pos += 1
        return chr(self.d[self.pos - 1])

    def putback(self):
        if not self.fail and self.pos > 0:
            self.pos -= 1


def chromosome_to_id(s):
    if s in ("X", "Y"):
        return 22 if s == "X" else 23
    digits = s[:len(s) - len(s.lstrip("+-0123456789"))] if s else ""
    if s == "" or digits != s:
        raise ValueError("Invalid chromosome: " + s)
    v = int(s) & 0xFFFFFFFF
    if v > 22:
        raise ValueError("Invalid chromosome: " + s)
    return (v - 1) & 0xFF


def read_map(map_file):
    if not map_file:
        return {}
    if not os.path.exists(map_file):
        raise ValueError("Map file does not exist")
    out = {}
    with open(map_file) as f:
        for line in f.read().split("\n"):
            if not line or line[0] == "#":
                continue
            cols = line.split("\t")
            if cols and cols[-1] == "":
                cols = cols[:-1]
            if len(cols) != 8:
                raise ValueError("Invalid map file")
            if cols[6] == "SEQ":
                continue
            out.setdefault(cols[1], []).append(((int(cols[2]) - 1) & 0xFFFFFFFF, int(cols[0]),
                                                "I" if cols[6] == "INS" else "D", chromosome_to_id(cols[3])))
    return out


def apply_map(entries, chr_data):
    i, out = 0, []
    for start, length, tr, *_ in entries:
        while i < start:
            out.append(chr_data[i])
            i += 1
        if tr == "D":
            out.extend([5] * length)
        else:
            i += length
    out.extend(chr_data[i:])
    return out


def read_contig(f):
    out = []
    while True:
        line = f.getline()
        if line is None:
            break
        out.extend(char_to_int(c) for c in line)
        if f.peek() == ">":
            break
    return out


def check_is_diploid(data):
    words = data.split()
    return bool(words) and b"maternal" in words[0]


def get_next_chromosome(f, mp, is_diploid, chr_data):
    """-> the new chr_data (the old one when the FASTA has no contig left)."""
    line = f.getline()
    if line is None:
        return chr_data
    chromosome = line[1] if len(line) > 1 else "\0"
    name = line[1:]
    tmp = read_contig(f)
    chr_data = apply_map(mp[name], tmp) if name in mp else tmp
    ch1 = f.get()
    ch2 = f.peek()
    if ch1 is not None:
        f.putback()
    if not is_diploid or (chromosome == "X" and ch2 == "Y") or chromosome == "Y":
        return [x | (x << 3) for x in chr_data]
    second = f.getline()
    if second is not None and second:
        name = second[1:]
    tmp = read_contig(f)
    pat = apply_map(mp[name], tmp) if name in mp else tmp
    if len(pat) != len(chr_data):
        raise ValueError("Maternal and paternal chromosome sizes don't match")
    return [(m << 3) | p for m, p in zip(chr_data, pat)]


# --- the calls ------------------------------------------------------------------------------------------------------

def is_same_genotype(a, b):
    return a == b or ((a >> 3) | ((a & 7) << 3)) == b


def is_homozygous(g):
    return (g & 7) == (g >> 3)


def get_differing_bases(ref, g):
    r1, r2 = sorted((INT_TO_CHAR[ref & 7], INT_TO_CHAR[ref >> 3]))
    g1, g2 = sorted((INT_TO_CHAR[g & 7], INT_TO_CHAR[g >> 3]))
    if g1 == r1 and g2 == r2:
        return []
    if g1 == r1:
        return [(r2, g2)]
    if g2 == r2:
        return [(r1, g1)]
    return [(r1, g1), (r2, g2)]


def _counts(n):
    return "\t%d %d %d %d \n" % tuple(n)


def vcf_lines(chr_idx, position, ref, g, nbases):
    if is_same_genotype(g, ref) or g == NO_GENOTYPE:
        return ""
    head = "%s\t%d\t.\t" % (id_to_chromosome(chr_idx), position)
    if is_homozygous(ref):
        alt, gt = INT_TO_CHAR[g & 7], "1/1"
        if not is_homozygous(g):
            alt += INT_TO_CHAR[g >> 3]
            gt = "0/1"
        return head + INT_TO_CHAR[ref & 7] + "\t" + alt + INFO_FORMAT + gt + _counts(nbases)
    return "".join(head + a + "\t" + b + INFO_FORMAT + "1/1" + _counts(nbases) for a, b in get_differing_bases(ref, g))


def calls(chromosomes, clusters, reference_genome, map_file="", hetero_prior=1e-3, theta=0.01):
    """chromosomes: per chromosome, a list of (position, [group_id << 2 | base, ...]).
    -> (per-cluster VCF bodies, common VCF body, mismatch per cell, loci per cell), or None for no cells."""
    if len(clusters) == 0:
        return None
    if not os.path.exists(reference_genome):
        raise ValueError("Reference genome does not exist")
    mp = read_map(map_file)
    num_clusters = int(max(clusters)) + 1
    with open(reference_genome, "rb") as fh:
        data = fh.read()
    f = Stream(data)
    diploid = check_is_diploid(data)
    chr_data = []
    vcfs = [""] * num_clusters
    common = []
    scores = [0] * len(clusters)
    loci = [0] * len(clusters)
    for chr_idx, chromosome in enumerate(chromosomes):
        chr_data = get_next_chromosome(f, mp, diploid, chr_data)
        for position, entries in chromosome:
            if ((position - 1) & 0xFFFFFFFF) >= len(chr_data):
                break
            total = [0, 0, 0, 0]
            nbases = {}
            for idb in entries:
                g, b = idb >> 2, idb & 3
                cl = int(clusters[g])
                nb = nbases.setdefault(cl, [0, 0, 0, 0])
                nb[b] = (nb[b] + 1) & 0xFFFF
                total[b] = (total[b] + 1) & 0xFFFF
                loci[g] += 1
            pooled = likely_homozygous(total, theta)
            ref = chr_data[position - 1]
            if pooled != NO_GENOTYPE and pooled != ref:
                new_base = pooled & 7
                ref_base = (ref >> 3) & 7 if (ref & 7) == new_base else ref & 7
                common.append("%s\t%d\t.\t%s\t%s%s1/1%s" % (id_to_chromosome(chr_idx), position, INT_TO_CHAR[ref_base],
                                                          INT_TO_CHAR[new_base], INFO_FORMAT, _counts(total)))
            # clusters without entries give NO_GENOTYPE with cov 0 and change nothing: only present ones matter
            genotypes, all_same, first = {}, True, NO_GENOTYPE
            for cl in sorted(nbases):
                g, cov = most_likely_genotype(nbases[cl], pooled != NO_GENOTYPE, hetero_prior, theta)
                genotypes[cl] = (g, cov)
                if g != NO_GENOTYPE and first == NO_GENOTYPE and cl > 0:
                    first = g
                if first != NO_GENOTYPE and cov > 0 and first != g:
                    all_same = False
            if all_same:
                common.append(vcf_lines(chr_idx, position, ref, genotypes.get(0, (NO_GENOTYPE, 0))[0], total))
                continue
            for cl in sorted(nbases):
                g = genotypes[cl][0]
                if pooled != NO_GENOTYPE and g == pooled:
                    continue
                vcfs[cl] += vcf_lines(chr_idx, position, ref, g, nbases[cl])
            for idb in entries:
                g_id, b = idb >> 2, idb & 3
                cl = int(clusters[g_id])
                g, cov = genotypes[cl]
                if g != NO_GENOTYPE and b != (g & 7) and b != (g >> 3) and cov > 9:
                    scores[g_id] += 1
    return vcfs, "".join(common), scores, loci


def preamble(reference, cluster):
    return ("##fileformat=VCFv4.2\n##fileDate=%s\n##source=SVC (Somatic Variant Caller)\n##reference=%s\n"
            "##cluster=%d\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tcluster-%d\n"
            % (time.ctime(), reference, cluster, cluster))


def format_score(mismatch, loci):
    if loci == 0:
        return "-nan"  # 0.0 / 0 under x86-64 libstdc++
    return "%g" % (mismatch / loci)


def write_files(chromosomes, clusters, reference_genome, out_dir, map_file="", hetero_prior=1e-3, theta=0.01):
    res = calls(chromosomes, clusters, reference_genome, map_file, hetero_prior, theta)
    if res is None:
        return
    os.makedirs(out_dir, exist_ok=True)
    vcfs, common, mismatch, loci = res
    for i, body in enumerate(vcfs):
        with open(os.path.join(out_dir, "cluster_%d.vcf" % i), "w") as f:
            f.write(preamble(reference_genome, i) + body)
    with open(os.path.join(out_dir, "common.vcf"), "w") as f:
        f.write(common)
    open(os.path.join(out_dir, "variant"), "w").close()
    with open(os.path.join(out_dir, "scores"), "w") as f:
        f.write(",".join(format_score(m, l) for m, l in zip(mismatch, loci)) + "\n")


def from_flat(p):
    """FlatPileup -> the `chromosomes` argument of calls()."""
    out = []
    for c in range(p.n_chr):
        chrom = []
        for l in range(int(p.chr_locus_off[c]), int(p.chr_locus_off[c + 1])):
            b, e = int(p.locus_entry_off[l]), int(p.locus_entry_off[l + 1])
            chrom.append((int(p.locus_pos[l]), [int(x) for x in p.id_base[b:e]]))
        out.append(chrom)
    return out


def strip_date(text):
    return "".join(line for line in text.splitlines(True) if not line.startswith("##fileDate="))


def read_dir(out_dir):
    """{file name: text without the ##fileDate line} of a result directory."""
    out = {}
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name)) as f:
            out[name] = strip_date(f.read())
    return out
