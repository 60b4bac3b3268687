"""Plain numpy / Python restatement of the per-cell allele counts at the called variants (include/secedo_variant.h,
"Per-cell allele counts"): from a FlatPileup, call records, the reference genotype per locus, the number of cells and
the selection to the sites and their masks, the (site, group) pairs, the per-site totals and the exact bytes of the five
files. Written for clarity, as tests/variant_ref.py is: one locus at a time, dictionaries, no tricks.
"""
import numpy as np

KIND_CLUSTER = 2
NAMES = ("cellSNP.tag.AD.mtx", "cellSNP.tag.DP.mtx", "cellSNP.tag.OTH.mtx", "cellSNP.base.vcf", "cellSNP.samples.tsv")
VCF_HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def bits(code):
    """The bases 0..3 among {code & 7, code >> 3}, as a mask; an N (5) adds nothing."""
    return sum(1 << b for b in {code & 7, code >> 3} if b < 4)


def masks(records, locus_ref, selection):
    """-> [(locus, ref_mask, alt_mask)] in ascending locus order. records: (locus, cluster, genotype, kind, counts)
    rows of a RECORD_DTYPE array (or tuples in that order)."""
    by_locus = {}
    for r in records:
        locus, genotype, kind = int(r[0]), int(r[2]), int(r[3])
        g, cluster = by_locus.get(locus, (0, False))
        by_locus[locus] = (g | bits(genotype), cluster or kind == KIND_CLUSTER)
    out = []
    for locus in sorted(by_locus):
        g, cluster = by_locus[locus]
        if selection == "cluster" and not cluster:
            continue
        rf = bits(int(locus_ref[locus]))
        alt, ref = g & ~rf, rf
        if alt == 0:
            alt, ref = g, rf & ~g
        out.append((locus, ref, alt))
    return out


def counts(p, sites):
    """-> (pairs [(site, group, ad, rd, oth)] by site then group, totals [(ad, rd, oth)] per site)."""
    pairs, totals = [], []
    for s, (locus, ref, alt) in enumerate(sites):
        per = {}
        for idb in p.id_base[int(p.locus_entry_off[locus]):int(p.locus_entry_off[locus + 1])]:
            g, bit = int(idb) >> 2, 1 << (int(idb) & 3)
            c = per.setdefault(g, [0, 0, 0])
            c[0 if alt & bit else 1 if ref & bit else 2] += 1
        tot = [0, 0, 0]
        for g in sorted(per):
            pairs.append((s, g, *per[g]))
            tot = [a + b for a, b in zip(tot, per[g])]
        totals.append(tuple(tot))
    return pairs, totals


def letters(mask):
    return ",".join("ACGT"[b] for b in range(4) if mask >> b & 1) or "N"


def chromosome_name(p, locus):
    c = 0  # the VCF writer's walk: the last chromosome keeps what lies past it
    while c + 1 < p.n_chr and locus >= int(p.chr_locus_off[c + 1]):
        c += 1
    return str(c + 1) if c < 22 else ("X" if c == 22 else "Y")


def mtx(n_sites, n_cells, triples):
    body = ["%d\t%d\t%d\n" % (s + 1, g + 1, v) for s, g, v in triples if v > 0]
    return ("%%%%MatrixMarket matrix coordinate integer general\n%%\n%d\t%d\t%d\n" % (n_sites, n_cells, len(body))
            + "".join(body)).encode()


def files(p, records, locus_ref, n_cells, selection, cell_names=None):
    """-> {file name: bytes} of the five files of the plain output."""
    sites = masks(records, locus_ref, selection)
    pairs, totals = counts(p, sites)
    vcf = VCF_HEADER
    for (locus, ref, alt), (ad, rd, oth) in zip(sites, totals):
        vcf += "%s\t%d\t.\t%s\t%s\t.\tPASS\tAD=%d;DP=%d;OTH=%d\n" % (
            chromosome_name(p, locus), int(p.locus_pos[locus]), letters(ref), letters(alt), ad, ad + rd, oth)
    names = ["cell_%d" % i for i in range(n_cells)] if cell_names is None else list(cell_names)
    return {NAMES[0]: mtx(len(sites), n_cells, [(s, g, ad) for s, g, ad, rd, oth in pairs]),
            NAMES[1]: mtx(len(sites), n_cells, [(s, g, ad + rd) for s, g, ad, rd, oth in pairs]),
            NAMES[2]: mtx(len(sites), n_cells, [(s, g, oth) for s, g, ad, rd, oth in pairs]),
            NAMES[3]: vcf.encode(),
            NAMES[4]: "".join(n + "\n" for n in names).encode()}


def as_arrays(sites, pairs, totals):
    """The restatement's lists in the dtypes secedo_amd.allele_counts returns."""
    from secedo_amd.variant import PAIR_DTYPE
    return {"site_locus": np.asarray([s[0] for s in sites], dtype=np.uint32),
            "ref_mask": np.asarray([s[1] for s in sites], dtype=np.uint8),
            "alt_mask": np.asarray([s[2] for s in sites], dtype=np.uint8),
            "totals": np.asarray(totals, dtype=np.uint32).reshape(-1, 3),
            "pairs": np.asarray(pairs, dtype=PAIR_DTYPE) if pairs else np.zeros(0, dtype=PAIR_DTYPE)}
