"""The inputs on which variant calling is pinned to the COMPILED reference (oracle/_ref/ref_variant), one list for
the CPU test (tests/test_variant_reference_cpu.py), the golden writer (oracle/gen_golden.py variant_cases) and the
GPU test (tests/test_gpu_variant_reference.py). Everything is seeded or built by hand; nothing here reads the
reference's tree.

A case is ``(name, chromosomes, clusters, fasta_text, map_text, prior, theta)``: `chromosomes` as tests/variant_ref.py
takes them (per chromosome a list of (position, [group_id << 2 | base, ...])), `clusters` a u16 array indexed by group
id, `fasta_text` the bytes of the reference genome, `map_text` the text of a Varsim map or "". These are the smallest
shapes at which each rule of the reference can still fail; every family says which rule it is there for.

`tuple_set()` is the set of count 4-tuples for the two decision functions, `SETTINGS` its twelve parameter sets.
"""
import hashlib
import os
import re

import numpy as np

from secedo_amd.pileup import FlatPileup

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_reference.npz")
GENOME_MARK = "<GENOME>"  # what normalise() puts in place of the genome's path in ##reference=
MISMATCH_WORDS = "Invalid reference genome. Maternal and paternal chromosome sizes don't match"

# (theta, prior, likely_homozygous_total) of the decision-function comparison
SETTINGS = [(theta, prior, lht) for theta in (1e-3, 0.01, 0.05) for prior in (1e-3, 0.2) for lht in (0, 1)]
EXHAUSTIVE_TOTAL = 30  # all count tuples with a + c + g + t <= this (the rules at coverage 9 and 16 lie inside)
WRAP_TUPLES = [(65535, 10, 0, 0), (32768, 32768, 9, 0), (65535, 1, 0, 0), (65535, 65535, 65535, 65535),
               (65527, 9, 9, 0), (40000, 25536, 0, 0), (0, 65535, 17, 0), (32768, 32767, 16, 1), (65530, 15, 0, 0),
               (21846, 21845, 21845, 9)]


# --- files ------------------------------------------------------------------------------------------------------------

def flat(chromosomes):
    """`chromosomes` -> FlatPileup (read ids: the entry's ordinal)."""
    chr_off, pos, off, idb = [0], [], [0], []
    for chrom in chromosomes:
        for p, entries in chrom:
            pos.append(p)
            idb.extend(entries)
            off.append(len(idb))
        chr_off.append(len(pos))
    idb = np.asarray(idb, dtype=np.uint32)
    return FlatPileup(np.asarray(chr_off), np.asarray(pos), np.asarray(off, dtype=np.uint64),
                      np.arange(len(idb), dtype=np.uint32), idb)


def write_flat(path, p, n_cells, wide=False):
    """The flat pileup file tests/cpp/variant_calling_test.cpp and oracle/ref_variant_driver.cpp read: u64 n_chr,
    n_loci, n_entries, n_cells, then the five arrays, id_base as u16 (`wide`: u32, which only the driver reads)."""
    idb = np.ascontiguousarray(p.id_base)
    if not wide and p.n_entries and int(idb.max()) > 0xFFFF:
        raise ValueError("a group id does not fit the u16 id_base of the flat file")
    with open(path, "wb") as f:
        np.asarray([p.n_chr, p.n_loci, p.n_entries, n_cells], dtype=np.uint64).tofile(f)
        np.ascontiguousarray(p.chr_locus_off, dtype=np.uint32).tofile(f)
        np.ascontiguousarray(p.locus_pos, dtype=np.uint32).tofile(f)
        np.ascontiguousarray(p.locus_entry_off, dtype=np.uint64).tofile(f)
        np.ascontiguousarray(p.read_ids, dtype=np.uint32).tofile(f)
        idb.astype(np.uint32 if wide else np.uint16).tofile(f)


def write_clusters(path, clusters):
    with open(path, "wb") as f:
        np.asarray([len(clusters)], dtype=np.uint64).tofile(f)
        np.ascontiguousarray(clusters, dtype=np.uint16).tofile(f)


def write_genome(case, directory):
    """The case's FASTA and map as files under `directory` -> (fasta path, map path or "")."""
    name, _, _, fasta_text, map_text, _, _ = case
    fasta = os.path.join(str(directory), name + ".fa")
    with open(fasta, "wb") as f:
        f.write(fasta_text)
    mp = ""
    if map_text:
        mp = os.path.join(str(directory), name + ".map")
        with open(mp, "w") as f:
            f.write(map_text)
    return fasta, mp


def normalise(text, genome):
    """A result file without what depends on the run: the ##fileDate line dropped, the genome's path in ##reference=
    replaced by GENOME_MARK (any other path stays and shows as a difference)."""
    out = []
    for line in text.splitlines(True):
        if line.startswith("##fileDate="):
            continue
        if line == "##reference=%s\n" % genome:
            line = "##reference=%s\n" % GENOME_MARK
        out.append(line)
    return "".join(out)


def run_reference(case, directory):
    """The compiled reference on one case -> (returncode, log, {file: normalised text})."""
    from oracle import bindings as ob
    name, chromosomes, clusters, _, _, prior, theta = case
    fasta, mp = write_genome(case, directory)
    pb, cb = os.path.join(str(directory), name + ".p.bin"), os.path.join(str(directory), name + ".c.bin")
    write_flat(pb, flat(chromosomes), len(clusters))
    write_clusters(cb, clusters)
    rc, log, files = ob.ref_variant_calling(pb, cb, fasta, mp, prior, theta, os.path.join(str(directory), name + ".ref"))
    return rc, log, {k: normalise(v, fasta) for k, v in files.items()}


def mismatch_message(log):
    """The reference's words for unequal maternal and paternal contigs, out of its coloured log ("" if absent)."""
    m = re.search(re.escape(MISMATCH_WORDS) + r" \(\d+ vs \d+\)", log)
    return m.group(0) if m else ""


# --- the decision functions' tuples -----------------------------------------------------------------------------------

def tuples_up_to(total):
    out = []
    for a in range(total + 1):
        for b in range(total + 1 - a):
            for c in range(total + 1 - a - b):
                for d in range(total + 1 - a - b - c):
                    out.append((a, b, c, d))
    return np.asarray(out, dtype=np.uint16)


_tuple_set = None


def tuple_set():
    """(n, 4) u16: every tuple with total <= EXHAUSTIVE_TOTAL, 3000 seeded ones below 250, 3000 over the whole u16
    range, and the hand-made tuples whose u16 sum or whose `cov - max` wraps."""
    global _tuple_set
    if _tuple_set is None:
        rng = np.random.default_rng(20261021)
        _tuple_set = np.concatenate([tuples_up_to(EXHAUSTIVE_TOTAL), rng.integers(0, 250, (3000, 4)).astype(np.uint16),
                                     rng.integers(0, 65536, (3000, 4)).astype(np.uint16),
                                     np.asarray(WRAP_TUPLES, dtype=np.uint16)])
        _tuple_set.setflags(write=False)
    return _tuple_set


def tuple_digest(counts):
    return hashlib.sha256(np.ascontiguousarray(counts, dtype=np.uint16).tobytes()).hexdigest()


# --- building blocks --------------------------------------------------------------------------------------------------

def _wrap_text(s, w=60):
    return "\n".join(s[i:i + w] for i in range(0, len(s), w))


def _haploid(seqs, names=None, w=60):
    names = names or ["chr%d" % (i + 1) for i in range(len(seqs))]
    return "".join(">%s\n%s\n" % (n, _wrap_text(s, w)) for n, s in zip(names, seqs)).encode()


def _diploid(pairs, names=None, w=60):
    names = names or [str(i + 1) for i in range(len(pairs))]
    return "".join(">%s_maternal\n%s\n>%s_paternal\n%s\n" % (n, _wrap_text(m, w), n, _wrap_text(p, w))
                   for n, (m, p) in zip(names, pairs)).encode()


def _random_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def _variant_of(rng, s, rate=0.15):
    return "".join(c if rng.random() >= rate else str(rng.choice(list("ACGT"))) for c in s)


def _entries(rng, by_cluster, groups_of, extra=()):
    """Entries with the given base counts per cluster, cells taken in turn from the cluster's groups, in a seeded
    order; `extra`: (group, base) pairs added as they are."""
    out = []
    for cl, counts in by_cluster.items():
        k = 0
        for base, n in enumerate(counts):
            for _ in range(n):
                out.append(groups_of[cl][k % len(groups_of[cl])] << 2 | base)
                k += 1
    out.extend(g << 2 | b for g, b in extra)
    return [int(x) for x in rng.permutation(np.asarray(out, dtype=np.int64))] if out else []


def _synthetic(rng, n_groups, n_clusters, lengths, n_chr, per_chr=15):
    """Seeded loci over `n_chr` chromosomes (the c-th within lengths[min(c, last)]) -> (chromosomes, clusters)."""
    clusters = rng.integers(0, n_clusters, n_groups).astype(np.uint16)
    clusters[:n_clusters] = np.arange(n_clusters)
    chromosomes = []
    for c in range(n_chr):
        length = lengths[min(c, len(lengths) - 1)]
        pos = np.sort(rng.choice(np.arange(1, length + 1), min(length, per_chr), replace=False)).tolist()
        chrom = []
        for p in pos:
            cov = int(rng.choice([3, 8, 12, 20, 30, 45, 64, 70]))
            alleles = {k: rng.choice(4, 2) if rng.random() < 0.3 else np.repeat(rng.integers(4), 2)
                       for k in range(n_clusters)}
            entries = []
            for g in rng.integers(0, n_groups, cov):
                b = int(rng.choice(alleles[int(clusters[g])]))
                if rng.random() < 0.03:
                    b = int(rng.integers(4))
                entries.append(int(g) << 2 | b)
            chrom.append((int(p), entries))
        chromosomes.append(chrom)
    return chromosomes, clusters


# --- wrap: u16 counts that wrap -----------------------------------------------------------------------------------------

WRAP_GROUPS = 1000  # groups 0..599 in cluster 1, 600..999 in cluster 2


def wrap():
    """One chromosome, clusters 1 and 2, three loci, 196 666 entries.
    position 1: 65 545 A in cluster 1, 20 C in cluster 2. Cluster 1's count and coverage wrap to 9: the `cov < 9` edge
        of most_likely_genotype (a call) and the `cov > 9` edge of the mismatch rule. Its line shows "9 0 0 0".
    position 2: 30 C in cluster 1, 65 536 A in cluster 2. Cluster 2's coverage wraps to 0: it counts as absent for
        all_same although it comes after a cluster with a call, so the locus is all_same; its cells still get the locus
        in `scores`. The pooled line shows "0 30 0 0".
    position 3: 65 510 A and 5 G in cluster 1, 20 C in cluster 2: 65 535 entries, nothing wraps (the control); the five
        G cells are mismatches."""
    clusters = np.where(np.arange(WRAP_GROUPS) < 600, 1, 2).astype(np.uint16)
    c1 = lambda n, base, start=0: (((np.arange(n) + start) % 600) << 2 | base).tolist()
    c2 = lambda n, base: ((600 + np.arange(n) % 400) << 2 | base).tolist()
    loci = [(1, c1(65545, 0) + c2(20, 1)),
            (2, c2(40000, 0) + c1(30, 1) + c2(25536, 0)),
            (3, c1(30000, 0) + c1(5, 2, 77) + c2(20, 1) + c1(35510, 0, 123))]
    return [("wrap", [loci], clusters, _haploid(["GGTACGT"]), "", 1e-3, 0.01)]


WRAP_EXPECT = {  # the precondition: lines of the recorded reference output with a wrapped count column
    "cluster_1.vcf": "1\t1\t.\tG\tA\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t1/1\t%d 0 0 0 \n" % (65545 - 65536),
    "common.vcf": "1\t2\t.\tG\tC\t.\t.\tVARIANT_OVERALL_TYPE=SNP\tGT\t1/1\t%d 30 0 0 \n" % (65536 - 65536),
}


# --- many_clusters ------------------------------------------------------------------------------------------------------

def many_clusters():
    """16 384 groups (the ceiling of the reference's 14 bits; group 16 383 is used) in 90 clusters, cells in cluster 0
    among them; 39 loci whose coverages cycle 70, 130, 1100, 20, 5, 300 (several 64-entry chunks per locus, more than
    64 clusters present at one locus), and a second chromosome with the first ten loci."""
    rng = np.random.default_rng(516)
    n_groups, n_clusters = 16384, 90
    clusters = rng.integers(0, n_clusters, n_groups).astype(np.uint16)
    clusters[:n_clusters] = np.arange(n_clusters)
    mat = _random_seq(rng, 60)
    pairs = [(mat, _variant_of(rng, mat)), (mat[::-1], _variant_of(rng, mat[::-1]))]
    chrom = []
    for p in range(1, 40):
        cov = [70, 130, 1100, 20, 5, 300][p % 6]
        groups = rng.integers(0, n_groups, cov)
        groups[0] = n_groups - 1
        alt = int(rng.integers(4))
        entries = [int(g) << 2 | (alt if clusters[g] % 3 == 0 else int(rng.integers(2)) if clusters[g] % 3 == 1 else 2)
                   for g in groups]
        chrom.append((p, entries))
    return [("many_clusters", [chrom, chrom[:10]], clusters, _diploid(pairs), "", 1e-3, 0.01)]


# --- ties: counts built to sit on each tie and threshold rule -------------------------------------------------------------

# groups of the ties cases: cluster 1 = 0..19, cluster 2 = 20..37 (38 and 39 are the two score cells), cluster 3 =
# 40..55, cluster 0 = 56..63
TIES_GROUPS = {1: list(range(0, 20)), 2: list(range(20, 38)), 3: list(range(40, 56)), 0: list(range(56, 64))}
TIES_CLUSTERS = np.asarray([1] * 20 + [2] * 20 + [3] * 16 + [0] * 8, dtype=np.uint16)
SCORE_CELL_COV9, SCORE_CELL_COV10 = 38, 39
T12 = (0, 0, 0, 12)  # the witness: cluster 1 calls T/T, so a later cluster without that call ends all_same
A12 = (12, 0, 0, 0)


def _ties_loci(theta):
    """(rule, maternal + paternal reference base, {cluster: (a, c, g, t)}, extra entries). The probe is cluster 2 unless
    the rule says otherwise: cluster 1 is evaluated first and has a call, so whatever cluster 2 gets is written."""
    t = {1e-3: 0, 0.01: 1, 0.05: 3}[theta]  # round(40 theta + sqrt(40 theta (1 - theta))): likely_homozygous at cov 40
    return [
        # most_likely_genotype: ties among the maxima (the highest base index is idx[3])
        ("two_maxima_AC", "GG", {1: T12, 2: (10, 10, 0, 0)}, ()),
        ("two_maxima_CG", "AA", {1: T12, 2: (0, 10, 10, 0)}, ()),
        ("two_maxima_AT", "GG", {1: (0, 12, 0, 0), 2: (10, 0, 0, 10)}, ()),
        ("three_maxima", "GG", {1: T12, 2: (6, 6, 6, 0)}, ()),
        ("four_maxima", "GG", {1: T12, 2: (4, 4, 4, 4)}, ()),
        ("n2_eq_n3_small", "GG", {1: T12, 2: (3, 3, 3, 0)}, ()),      # homozygous wins only under a tiny prior
        ("n2_eq_n3_two", "GG", {1: T12, 2: (5, 5, 0, 0)}, ()),
        ("n2_lt_n3_small", "GG", {1: T12, 2: (4, 3, 2, 0)}, ()),
        ("n2_eq_n1_hetero", "GG", {1: T12, 2: (10, 5, 5, 0)}, ()),
        # the +-1 sigma test of a heterozygous call, in integers: 4 d^2 against s = n3 + n2
        ("four_d2_eq_s", "GG", {1: T12, 2: (10, 6, 0, 0)}, ()),       # d = 2, s = 16: `<=` holds, `<` does not
        ("one_sigma_inside", "GG", {1: T12, 2: (9, 7, 0, 0)}, ()),
        ("one_sigma_outside", "GG", {1: T12, 2: (11, 5, 0, 0)}, ()),
        ("odd_sum_inside", "GG", {1: T12, 2: (10, 7, 0, 0)}, ()),     # mean = 8 by integer division
        ("odd_sum_outside", "GG", {1: T12, 2: (11, 6, 0, 0)}, ()),
        # coverage thresholds
        ("cov15_hetero", "GG", {1: T12, 2: (8, 7, 0, 0)}, ()),
        ("cov16_hetero", "GG", {1: T12, 2: (8, 8, 0, 0)}, ()),
        ("cov8_no_call", "GG", {1: T12, 2: (8, 0, 0, 0)}, ()),
        ("cov9_call", "GG", {1: T12, 2: (9, 0, 0, 0)}, ()),
        ("cov9_no_mismatch", "GG", {1: T12, 2: (8, 0, 0, 0)}, ((SCORE_CELL_COV9, 1),)),
        ("cov10_mismatch", "GG", {1: T12, 2: (9, 0, 0, 0)}, ((SCORE_CELL_COV10, 1),)),
        ("pooled_cov8", "GG", {1: (5, 0, 0, 0), 2: (3, 0, 0, 0)}, ()),
        ("pooled_cov9", "GG", {1: (5, 0, 0, 0), 2: (4, 0, 0, 0)}, ()),
        # likely_homozygous_total lets clusters below coverage 9 call when max >= cov - 1
        ("lht_cov8", "GG", {3: (28, 0, 0, 0), 1: (8, 0, 0, 0), 2: (0, 1, 0, 0)}, ()),
        # (cluster 2 comes before cluster 3, whose call is the pooled one: a call of cluster 2 ends all_same and is
        # written, no call leaves the locus all_same; four other bases among 49 are pooled-homozygous at theta 0.05 only)
        ("lht_max_eq_cov_minus_1", "CC", {3: (45, 0, 0, 0), 2: (0, 0, 3, 1)}, ()),
        ("lht_max_below_cov_minus_1", "CC", {3: (45, 0, 0, 0), 2: (0, 0, 2, 2)}, ()),
        ("lht_tie_at_cov2", "CC", {3: (45, 0, 0, 0), 2: (0, 0, 1, 1)}, ()),
        # cov - max at the likely_homozygous threshold of coverage 40 and one above it
        ("threshold_at", "GG", {1: (20, 0, 0, 0), 2: (20 - t, t, 0, 0)}, ()),
        ("threshold_above", "GG", {1: (20, 0, 0, 0), 2: (19 - t, t + 1, 0, 0)}, ()),
        # the pooled call against the reference base
        ("pooled_eq_ref", "AA", {1: (5, 0, 0, 0), 2: (4, 0, 0, 0)}, ()),
        ("pooled_ne_ref", "CC", {1: (5, 0, 0, 0), 2: (4, 0, 0, 0)}, ()),
        ("pooled_ref_maternal", "AG", {1: (5, 0, 0, 0), 2: (4, 0, 0, 0)}, ()),
        ("pooled_ref_paternal", "GA", {1: (5, 0, 0, 0), 2: (4, 0, 0, 0)}, ()),
        # a heterozygous reference: get_differing_bases
        ("het_ref_two_lines", "AG", {1: T12, 2: A12}, ()),
        ("het_ref_same_genotype", "AG", {1: T12, 2: (8, 0, 8, 0)}, ()),
        ("het_ref_first_equal", "AG", {1: T12, 2: (8, 8, 0, 0)}, ()),
        ("het_ref_second_equal", "CT", {1: (0, 0, 12, 0), 2: (8, 0, 0, 8)}, ()),
        ("ref_n", "NN", {1: T12, 2: A12}, ()),
        # all_same and first_genotype
        ("no_call_after_call", "GG", {1: A12, 2: (3, 3, 3, 0)}, ()),
        ("no_call_before_call", "GG", {1: (3, 3, 3, 0), 2: A12, 3: A12}, ()),
        ("differs_after_first", "GG", {1: (3, 3, 3, 0), 2: A12, 3: T12}, ()),
        ("first_skips_cluster0", "GG", {0: T12, 1: A12, 2: A12}, ()),
        ("cluster0_after_nothing", "GG", {0: T12, 1: (3, 3, 3, 0)}, ()),
    ]


TIES_SETTINGS = [("ties_theta_0.001", 1e-3, 1e-3), ("ties_theta_0.01", 1e-3, 0.01), ("ties_theta_0.05", 1e-3, 0.05),
                 ("ties_prior_1e-9", 1e-9, 0.01)]  # (name, prior, theta)


def ties_rules(theta=0.01):
    return [r[0] for r in _ties_loci(theta)]


def ties():
    """About 40 loci of at most 64 entries on one diploid contig pair, position = 1 + the rule's place in
    _ties_loci; under theta 1e-3, 0.01 and 0.05 at prior 1e-3, and at prior 1e-9 where a homozygous call can win
    with n2 == n3. TIES_EXPECT says what the reference writes at every locus."""
    out = []
    for name, prior, theta in TIES_SETTINGS:
        rng = np.random.default_rng(77)
        loci = _ties_loci(theta)
        mat, pat = "".join(l[1][0] for l in loci), "".join(l[1][1] for l in loci)
        chrom = [(i + 1, _entries(rng, by_cluster, TIES_GROUPS, extra)) for i, (_, _, by_cluster, extra) in enumerate(loci)]
        assert max(len(e) for _, e in chrom) <= 64
        out.append((name, [chrom], TIES_CLUSTERS, _diploid([(mat, pat)]), "", prior, theta))
    return out


def lines_at(files, position):
    """What the result files say at one position of chromosome 1: "file:REF>ALT:GT" joined by ';', files in order."""
    out = []
    for name in sorted(files):
        if not name.endswith(".vcf"):
            continue
        for line in files[name].splitlines():
            c = line.split("\t")
            if line and line[0] != "#" and c[0] == "1" and c[1] == str(position):
                out.append("%s:%s>%s:%s" % (name[:-4], c[3], c[4], c[9]))
    return ";".join(out)


# rule -> what the reference writes there under (theta 1e-3, theta 0.01, theta 0.05, prior 1e-9), or one string when the
# four agree. Worked out from the rule each locus is named for, and equal to the compiled reference's files
# (tests/test_variant_reference_cpu.py).
_W = "cluster_1:G>T:1/1"  # the witness' own line
_HOMO_A = "cluster_1:G>T:1/1;cluster_2:G>A:1/1"
TIES_EXPECT = {
    "two_maxima_AC": "cluster_1:G>T:1/1;cluster_2:G>AC:0/1",
    "two_maxima_CG": "cluster_1:A>T:1/1;cluster_2:A>CG:0/1",
    "two_maxima_AT": "cluster_1:G>C:1/1;cluster_2:G>AT:0/1",
    "three_maxima": _W,
    "four_maxima": _W,
    "n2_eq_n3_small": _W,  # heterozygous wins and n2 == n1; under the tiny prior homozygous wins and n2 == n3
    "n2_eq_n3_two": _W,
    "n2_lt_n3_small": (_W, _W, _W, _HOMO_A),
    "n2_eq_n1_hetero": (_W, _W, _W, _HOMO_A),
    "four_d2_eq_s": _W,
    "one_sigma_inside": "cluster_1:G>T:1/1;cluster_2:G>CA:0/1",
    "one_sigma_outside": (_W, _W, _W, _HOMO_A),
    "odd_sum_inside": "cluster_1:G>T:1/1;cluster_2:G>CA:0/1",
    "odd_sum_outside": _W,
    "cov15_hetero": _W,
    "cov16_hetero": "cluster_1:G>T:1/1;cluster_2:G>AC:0/1",
    "cov8_no_call": _W,
    "cov9_call": _HOMO_A,
    "cov9_no_mismatch": _HOMO_A,
    "cov10_mismatch": _HOMO_A,
    "pooled_cov8": "",
    "pooled_cov9": "common:G>A:1/1",
    "lht_cov8": ("", "cluster_2:G>C:1/1;common:G>A:1/1", "cluster_2:G>C:1/1;common:G>A:1/1",
                 "cluster_2:G>C:1/1;common:G>A:1/1"),
    "lht_max_eq_cov_minus_1": ("", "", "cluster_2:C>G:1/1;common:C>A:1/1", ""),
    "lht_max_below_cov_minus_1": ("", "", "common:C>A:1/1", ""),
    "lht_tie_at_cov2": ("", "", "cluster_2:C>T:1/1;common:C>A:1/1", ""),
    "threshold_at": "common:G>A:1/1",
    "threshold_above": "",
    "pooled_eq_ref": "",
    "pooled_ne_ref": "common:C>A:1/1",
    "pooled_ref_maternal": "common:G>A:1/1",
    "pooled_ref_paternal": "common:G>A:1/1",
    "het_ref_two_lines": "cluster_1:A>T:1/1;cluster_1:G>T:1/1;cluster_2:G>A:1/1",
    "het_ref_same_genotype": "cluster_1:A>T:1/1;cluster_1:G>T:1/1",
    "het_ref_first_equal": "cluster_1:A>T:1/1;cluster_1:G>T:1/1;cluster_2:G>C:1/1",
    "het_ref_second_equal": "cluster_1:C>G:1/1;cluster_1:T>G:1/1;cluster_2:C>A:1/1",
    "ref_n": "cluster_1:N>T:1/1;cluster_2:N>A:1/1",
    "no_call_after_call": "cluster_1:G>A:1/1",
    "no_call_before_call": "",
    "differs_after_first": "cluster_2:G>A:1/1;cluster_3:G>T:1/1",
    "first_skips_cluster0": "common:G>T:1/1",
    "cluster0_after_nothing": "common:G>T:1/1",
}
TIES_SCORES = {SCORE_CELL_COV9: "0", SCORE_CELL_COV10: "1"}  # the two score cells' entries of `scores`


def ties_expected(case_name, rule):
    e = TIES_EXPECT[rule]
    return e if isinstance(e, str) else e[[s[0] for s in TIES_SETTINGS].index(case_name)]


# --- fasta_quirks -------------------------------------------------------------------------------------------------------

def _quirk_texts(rng):
    """name -> (fasta bytes, contig lengths as the reference sees them, number of chromosomes)"""
    a, b = _random_seq(rng, 30), _random_seq(rng, 26)
    a2, b2 = _variant_of(rng, a), _variant_of(rng, b)
    lower = lambda s: "".join(c.lower() if i % 3 else c for i, c in enumerate(s))
    with_n = lambda s: s[:7] + "NNNN" + s[11:20] + "n" + s[21:]
    iupac = lambda s: s[:5] + "RYKM" + s[9:14] + "SWBDHVU" + s[21:25] + "-*" + s[27:]
    x, y = _random_seq(rng, 24), _random_seq(rng, 20)
    return {
        "lowercase": (_diploid([(lower(a), lower(a2)), (lower(b), b2)], w=11), [30, 26], 2),
        "n_bases": (_haploid([with_n(a), with_n(b)], w=11), [30, 26], 2),
        "iupac": (_haploid([iupac(a), iupac(b)], w=11), [30, 26], 2),
        # every line ends in '\r', which is read as one more base (N): lines of 10 + 1
        "crlf": (_diploid([(a, a2), (b, b2)], w=10).replace(b"\n", b"\r\n"), [33, 29], 2),
        "blank_lines": ((">chr1\n%s\n\n%s\n\n>chr2\n\n%s\n%s\n\n" % (a[:12], a[12:], b[:20], b[20:])).encode(),
                        [30, 26], 2),
        "no_final_newline": (_haploid([a, b], w=11)[:-1], [30, 26], 2),
        "one_contig_two_chromosomes": (_haploid([a], w=11), [30, 30], 2),
        "empty_contig": ((">chr1\n\n>chr2\n%s\n" % _wrap_text(b, 11)).encode(), [0, 26], 2),
        "male_xy": (_diploid([(a, a2)], w=11) + (">X_maternal\n%s\n>Y_paternal\n%s\n" % (_wrap_text(x, 11),
                                                                                         _wrap_text(y, 11))).encode(),
                    [30, 24, 20], 3),
        "fewer_contigs": (_diploid([(a, a2)], w=11), [30, 30, 30], 3),
    }


QUIRK_MAP = ("2\tchr1\t5\t1\t5\t+\tDEL\t.\n"
             "# a comment\n"
             "3\tchr1\t12\t1\t10\t+\tINS\t.\n"
             "4\tchr1\t20\t1\t15\t+\tSEQ\t.\n"
             "1\tchr2\t3\t2\t3\t+\tINS\t.\n")


def fasta_quirks():
    """The FASTA texts the reference accepts and reads in its own way, each under two or three chromosomes of about
    15 loci over 40 groups in clusters 0..3; and the positions that end a chromosome: 0 (position - 1 wraps) and one
    past the contig's end, each followed by a locus that is then never read."""
    rng = np.random.default_rng(909)
    out = []
    for name, (text, lengths, n_chr) in _quirk_texts(rng).items():
        chroms, clusters = _synthetic(rng, 40, 4, [max(n, 12) for n in lengths], n_chr)
        out.append(("fasta_" + name, chroms, clusters, text, "", 1e-3, 0.01))
    a, b = _random_seq(rng, 30), _random_seq(rng, 26)
    plain = _haploid([a, b], w=11)
    chroms, clusters = _synthetic(rng, 40, 4, [30, 26], 2)
    chroms[1] = [(0, chroms[1][0][1])] + chroms[1]
    out.append(("fasta_position_zero", chroms, clusters, plain, "", 1e-3, 0.01))
    chroms, clusters = _synthetic(rng, 40, 4, [30, 26], 2)
    chroms[0] = chroms[0][:8] + [(35, chroms[0][8][1]), (3, chroms[0][9][1])] + chroms[0][10:]
    out.append(("fasta_past_end_then_smaller", chroms, clusters, plain, "", 1e-3, 0.01))
    chroms, clusters = _synthetic(rng, 40, 4, [29, 25], 2)  # the map: chr1 30 + 2 - 3, chr2 26 - 1
    out.append(("fasta_mapped", chroms, clusters, plain, QUIRK_MAP, 1e-3, 0.01))
    return out


# --- extremes -----------------------------------------------------------------------------------------------------------

def extremes():
    rng = np.random.default_rng(4242)
    a, b = _random_seq(rng, 30), _random_seq(rng, 26)
    text = _diploid([(a, _variant_of(rng, a)), (b, _variant_of(rng, b))], w=11)
    out = []
    chroms, clusters = _synthetic(rng, 40, 4, [30, 26], 2)
    out.append(("extreme_all_cluster_0", chroms, np.zeros(40, np.uint16), text, "", 1e-3, 0.01))
    out.append(("extreme_single_cluster_1", chroms, np.ones(40, np.uint16), text, "", 1e-3, 0.01))
    # theta 0.4: likely_homozygous holds with two equal maxima (5, 5, 0, 0): max_element takes the LOWEST index, A
    tie = (1, [g << 2 | (0 if g < 5 else 1) for g in range(10)])
    tie_clusters = clusters.copy()
    tie_clusters[:10] = [1] * 5 + [2] * 5
    out.append(("extreme_theta_0.4", [[tie] + [l for l in chroms[0] if l[0] > 1], chroms[1]], tie_clusters, text, "",
                1e-3, 0.4))
    out.append(("extreme_prior_0.5", chroms, clusters, text, "", 0.5, 0.01))
    # 24 chromosomes: the 23rd and 24th are written as X and Y
    seqs = [_random_seq(rng, 12, "AC") for _ in range(24)]
    chroms24 = []
    for c in range(24):
        loci = [(1 + c % 5, [g << 2 | 2 for g in range(12)] + [(20 + g) << 2 | 3 for g in range(12)]),
                (7 + c % 3, [int(g) << 2 | int(rng.integers(4)) for g in rng.integers(0, 40, 25)])]
        chroms24.append(loci)
    cl24 = np.asarray([1] * 20 + [2] * 20, dtype=np.uint16)
    out.append(("extreme_24_chromosomes", chroms24, cl24, _haploid(seqs), "", 1e-3, 0.01))
    return out


# --- refused ------------------------------------------------------------------------------------------------------------

def refused():
    """Diploid genomes whose maternal and paternal contigs differ in length: the reference logs its error and calls
    exit(1), after the preambles are written. The second text has no paternal contig at all (length 0)."""
    locus = [[(1, [g << 2 for g in range(12)])]]
    clusters = np.ones(12, dtype=np.uint16)
    return [("refused_lengths_differ_by_one", locus, clusters, b">1_maternal\nACGTA\n>1_paternal\nACGT\n", "", 1e-3, 0.01),
            ("refused_missing_paternal", locus, clusters, b">1_maternal\nACGTA\n", "", 1e-3, 0.01)]


REFUSED_EXPECT = {"refused_lengths_differ_by_one": MISMATCH_WORDS + " (5 vs 4)",
                  "refused_missing_paternal": MISMATCH_WORDS + " (5 vs 0)"}


_cases = None


def accepted():
    """Every case the reference runs to its end, built once."""
    global _cases
    if _cases is None:
        _cases = wrap() + many_clusters() + ties() + fasta_quirks() + extremes()
    return _cases


def accepted_names():
    return ["wrap", "many_clusters"] + [s[0] for s in TIES_SETTINGS] + \
        ["fasta_" + k for k in ("lowercase", "n_bases", "iupac", "crlf", "blank_lines", "no_final_newline",
                                "one_contig_two_chromosomes", "empty_contig", "male_xy", "fewer_contigs",
                                "position_zero", "past_end_then_smaller", "mapped")] + \
        ["extreme_" + k for k in ("all_cluster_0", "single_cluster_1", "theta_0.4", "prior_0.5", "24_chromosomes")]


def case_named(name):
    for c in accepted() + refused():
        if c[0] == name:
            return c
    raise KeyError(name)


# --- the recorded reference results (tests/golden/variant_reference.npz) ------------------------------------------------

def golden_key(case_name, file_name):
    return "file|%s|%s" % (case_name, file_name)


def golden_arrays(results, refusals, tuples):
    """The arrays of the golden file. results: {case: {file: text}}; refusals: {case: (status, message)}; tuples:
    (digest, hom u8[3, n] per theta, gen u8[12, n] per setting, cov u16[n])."""
    arrays = {}
    for case, files in results.items():
        for name, text in files.items():
            arrays[golden_key(case, name)] = np.frombuffer(text.encode(), dtype=np.uint8)
    arrays["refused_names"] = np.array(sorted(refusals))
    arrays["refused_status"] = np.array([refusals[k][0] for k in sorted(refusals)], dtype=np.int32)
    arrays["refused_message"] = np.array([refusals[k][1] for k in sorted(refusals)])
    digest, hom, gen, cov = tuples
    arrays.update(tuples_digest=np.array(digest), tuples_hom=hom, tuples_gen=gen, tuples_cov=cov)
    return arrays


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_files(case_name):
    """{file: normalised text} the reference wrote for one case, from the golden file."""
    prefix = golden_key(case_name, "")
    return {k[len(prefix):]: v.tobytes().decode() for k, v in golden().items() if k.startswith(prefix)}


def reference_tuples(scratch_dir):
    """The compiled reference's decision functions on tuple_set() under SETTINGS -> golden_arrays' `tuples`."""
    from oracle import bindings as ob
    counts = tuple_set()
    hom, gen, cov = {}, [], None
    for theta, prior, lht in SETTINGS:
        h, g, c = ob.ref_variant_genotypes(counts, lht, prior, theta, scratch_dir)
        assert theta not in hom or np.array_equal(hom[theta], h)  # likely_homozygous depends on theta alone
        assert cov is None or np.array_equal(cov, c)
        hom[theta], cov = h, c
        gen.append(g)
    return tuple_digest(counts), np.stack([hom[t] for t in (1e-3, 0.01, 0.05)]), np.stack(gen), cov
