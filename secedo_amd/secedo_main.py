"""``python -m secedo_amd.secedo_main``: the reference's ``secedo`` executable (secedo_main.cpp) on the GPU path.

``secedo -i <pileup file or directory> -o <output directory> [flags]``: reads the pileup files (binary ``.bin``
straight into HBM with the GPU loader, text ``.pileup`` through the host reader), runs the divide_cluster recursion
on the resident pileup, writing the reference's per-level files into -o, and calls variants when
--reference_genome is given. Flags, defaults and validators are the reference's, in the gflags spellings
(--f=v, --f v, -f v, --flag, --noflag, --flag=false). Flag and file-name checks run before torch is imported.
Departures: two input files for one chromosome and a --clustering file whose length is not the cell count are
errors (exit 1); --num_threads only sizes host pools (at most 16). --reference_genome may be plain FASTA, bgzip
(BGZF) or plain gzip (.fa.gz works; the kind is told by content); --fasta_route host|device (default: the
environment SECEDO_FASTA, else host) says where its parse and per-locus gather run, see secedo_amd/variant.py.
--vcf_output plain|bgzf (default: the environment SECEDO_VCF, else plain) says whether the VCF files are written as
text by the host or as bgzip-compressed .vcf.gz, formatted and deflated on the GPU. --vcf_index none|tbi (default: the
environment SECEDO_VCF_INDEX, else none) adds <file>.vcf.gz.tbi, the tabix index, beside each .vcf.gz; it needs
--vcf_output bgzf. --allele_counts none|all|cluster (default: the environment SECEDO_ALLELE_COUNTS, else none) adds
<-o>/allele_counts/: the per-cell alternate / total / other read counts at the called variants as sparse matrices
(cellSNP.tag.AD.mtx, .DP.mtx, .OTH.mtx), their sites (cellSNP.base.vcf) and cells (cellSNP.samples.tsv, the names from
--cell_names <file> or cell_<i>); it needs --reference_genome.
"""
from __future__ import annotations

import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

USAGE = "secedo -i <input_dir> -o <output_dir> arguments"
DEFAULT_CHROMOSOMES = ",".join([str(c) for c in range(1, 23)] + ["X"])
N_SLOTS = 24
MAX_POOL = 16

# name -> (kind, default); kinds: str, uint, double, bool
FLAGS: Dict[str, Tuple[str, object]] = {
    "i": ("str", "./"),
    "o": ("str", "./"),
    "chromosomes": ("str", DEFAULT_CHROMOSOMES),
    "pos_file": ("str", ""),
    "merge_count": ("uint", 1),
    "merge_file": ("str", ""),
    "max_cell_count": ("uint", 10_000),
    "max_coverage": ("uint", 100),
    "seq_error_rate": ("double", 0.01),
    "mutation_rate": ("double", 0.01),
    "homozygous_filtered_rate": ("double", 0.5),
    "heterozygous_prob": ("double", 1e-3),
    "clustering_type": ("str", "SPECTRAL6"),
    "termination": ("str", "BIC"),
    "normalization": ("str", "ADD_MIN"),
    "expectation_maximization": ("bool", False),
    "min_cluster_size": ("uint", 100),
    "tumor_purity": ("uint", 5),
    "arma_kmeans": ("bool", False),
    "reference_genome": ("str", ""),
    "map_file": ("str", ""),
    "fasta_route": ("str", ""),
    "vcf_output": ("str", ""),
    "vcf_index": ("str", ""),
    "allele_counts": ("str", ""),
    "cell_names": ("str", ""),
    "clustering": ("str", ""),
    "compute_read_stats": ("bool", False),
    "num_threads": ("uint", 8),
    "log_level": ("str", "trace"),
    "labels_file": ("str", ""),
}


class UsageError(Exception):
    """A command line the reference rejects: printed, exit status 1."""


class Flags(dict):
    __getattr__ = dict.__getitem__


def usage() -> str:
    lines = [USAGE, "", "Flags:"]
    for name, (kind, default) in FLAGS.items():
        lines.append("  -%s (%s) default: %r" % (name, kind, default))
    lines += ["", "--reference_genome takes plain FASTA, bgzip (BGZF) or plain gzip: genome.fa.gz works as it is.",
              "--fasta_route host|device: where the FASTA is parsed (default: SECEDO_FASTA, else host; BGZF: device).",
              "--vcf_output plain|bgzf: cluster_<i>.vcf / common.vcf as text, or as .vcf.gz compressed on the GPU "
              "(default: SECEDO_VCF, else plain).",
              "--vcf_index none|tbi: with --vcf_output bgzf, a tabix index <file>.vcf.gz.tbi beside each file "
              "(default: SECEDO_VCF_INDEX, else none).",
              "--allele_counts none|all|cluster: with --reference_genome, per-cell allele counts at the called variants "
              "under <-o>/allele_counts/ (sites x cells matrices AD, DP, OTH as Matrix Market, the sites as a VCF, the "
              "cells as a list); all: every locus with a call, cluster: the loci where clusters differ (default: "
              "SECEDO_ALLELE_COUNTS, else none).",
              "--cell_names <file>: one name per line for cellSNP.samples.tsv (default: cell_<i>)."]
    return "\n".join(lines)


def _convert(name: str, kind: str, text: str):
    try:
        if kind == "str":
            return text
        if kind == "bool":
            t = text.lower()
            if t in ("true", "t", "yes", "y", "1"):
                return True
            if t in ("false", "f", "no", "n", "0"):
                return False
            raise ValueError(text)
        if kind == "uint":
            v = int(text, 10)
            if v < 0 or v >= 1 << 32:
                raise ValueError(text)
            return v
        return float(text)
    except ValueError:
        raise UsageError("ERROR: illegal value '%s' specified for %s flag '%s'" % (text, kind, name)) from None


def parse_flags(argv: Sequence[str]) -> Flags:
    """gflags parsing: --f=v, -f=v, --f v, -f v, a bare --flag or --noflag for booleans, --flag=false.
    Arguments that are not flags are ignored, as ParseCommandLineFlags leaves them; '--' ends the flags."""
    out = Flags({k: d for k, (_, d) in FLAGS.items()})
    args = list(argv)
    i = 0
    while i < len(args):
        a = args[i]
        i += 1
        if a == "--":
            break
        if not a.startswith("-") or a == "-":
            continue
        body = a[2:] if a.startswith("--") else a[1:]
        name, eq, value = body.partition("=")
        if name not in FLAGS and name.startswith("no") and name[2:] in FLAGS and FLAGS[name[2:]][0] == "bool" \
                and not eq:
            out[name[2:]] = False
            continue
        if name not in FLAGS:
            raise UsageError("ERROR: unknown command line flag '%s'" % name)
        kind = FLAGS[name][0]
        if not eq:
            if kind == "bool":
                out[name] = True
                continue
            if i >= len(args):
                raise UsageError("ERROR: flag '%s' is missing its argument" % a)
            value = args[i]
            i += 1
        out[name] = _convert(name, kind, value)
    return out


def validate(f: Flags) -> None:
    """The reference's DEFINE_validator checks, and --arma_kmeans with SPECTRAL* (rejected by the library)."""
    if f.clustering_type not in ("FIEDLER", "SPECTRAL2", "SPECTRAL6"):
        raise UsageError("Invalid value for --clustering_type: %s.\nShould be one of FIEDLER, SPECTRAL2, SPECTRAL6"
                         % f.clustering_type)
    if f.termination not in ("AIC", "BIC"):
        raise UsageError("Invalid value for --termination: %s.\nShould be one of AIC, BIC" % f.termination)
    if f.normalization not in ("ADD_MIN", "EXPONENTIATE", "SCALE_MAX_1"):
        raise UsageError("Invalid value for --normalization: %s.\nShould be one of ADD_MIN, EXPONENTIATE, "
                         "SCALE_MAX_1" % f.normalization)
    if f.fasta_route not in ("", "host", "device"):
        raise UsageError("Invalid value for --fasta_route: %s.\nShould be one of host, device" % f.fasta_route)
    if f.vcf_output not in ("", "plain", "bgzf"):
        raise UsageError("Invalid value for --vcf_output: %s.\nShould be one of plain, bgzf" % f.vcf_output)
    if f.vcf_index not in ("", "none", "tbi"):
        raise UsageError("Invalid value for --vcf_index: %s.\nShould be one of none, tbi" % f.vcf_index)
    if f.vcf_index == "tbi" and (f.vcf_output or os.environ.get("SECEDO_VCF") or "plain") != "bgzf":
        raise UsageError("--vcf_index tbi indexes the compressed output only: add --vcf_output bgzf")
    if f.allele_counts not in ("", "none", "all", "cluster"):
        raise UsageError("Invalid value for --allele_counts: %s.\nShould be one of none, all, cluster" % f.allele_counts)
    if f.allele_counts in ("all", "cluster") and not f.reference_genome:
        raise UsageError("--allele_counts counts at the called variants: add --reference_genome")
    if f.cell_names and not os.path.exists(f.cell_names):
        raise UsageError("Cannot find cell names file: " + f.cell_names)
    if not 1 <= f.tumor_purity <= 5:
        raise UsageError("Invalid value for --tumor_purity: %d.\nShould be 1,2,3,4, or 5" % f.tumor_purity)
    if f.arma_kmeans and f.clustering_type != "FIEDLER":
        raise UsageError("--arma_kmeans is only supported with --clustering_type=FIEDLER")
    if f.merge_count == 0:
        raise UsageError("Invalid value for --merge_count: 0")


def chromosome_to_id(chromosome: str) -> int:
    """1..22 -> 0..21, X -> 22, Y -> 23 (util.cpp:143-160)."""
    if chromosome == "X":
        return 22
    if chromosome == "Y":
        return 23
    if chromosome.isdigit() and 1 <= int(chromosome) <= 22:
        return int(chromosome) - 1
    raise UsageError("Invalid chromosome: %s. Must be 1..22, X, Y" % chromosome)


def id_to_chromosome(c: int) -> str:
    return str(c + 1) if c < 22 else ("X" if c == 22 else "Y")


def get_chromosome(path: str) -> int:
    """<prefix>_<chromosome>.<ext>.<ext> -> chromosome id (spectral_clustering.cpp:301-309): the file name with
    two extensions stripped must split into exactly two '_' parts."""
    name = os.path.splitext(os.path.splitext(os.path.basename(path))[0])[0]
    parts = name.split("_")
    if len(parts) != 2:
        raise UsageError("Invalid pileup filename %s. Must be <bla>_chromosome.*" % path)
    return chromosome_to_id(parts[1])


def get_files(path: str, extension: str) -> List[str]:
    found = []
    for root, _dirs, names in os.walk(path):
        found.extend(os.path.join(root, n) for n in names if os.path.splitext(n)[1] == extension)
    return found


def input_files(path: str) -> List[str]:
    """A file, or a directory searched recursively for .bin files, else .pileup files; sorted."""
    if not os.path.isdir(path):
        return [path]
    files = get_files(path, ".bin") or get_files(path, ".pileup")
    return sorted(files)


def chr_to_idx(chromosome: str) -> int:
    if chromosome == "X":
        return 22
    if chromosome == "Y":
        return 23
    if not chromosome.isdigit():
        return 255
    return int(chromosome) - 1


def read_positions(path: str) -> List[List[int]]:
    """--pos_file (util.cpp:104-141): chromosome TAB position per line; '#' lines and chromosomes past Y are
    skipped; one sorted list per chromosome id up to the largest one present."""
    if not os.path.exists(path):
        raise UsageError("Could not find positions file: %s" % path)
    result: List[List[int]] = []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith("#"):
                continue
            cols = line.split("\t")
            c = chr_to_idx(cols[0])
            if c > 23:
                continue
            try:
                pos = int(cols[1])
            except (IndexError, ValueError):
                raise UsageError("Invalid line in %s: %s" % (path, line)) from None
            while len(result) <= c:
                result.append([])
            result[c].append(pos)
    for v in result:
        v.sort()
    return result


def read_clustering(path: str) -> List[int]:
    if not os.path.exists(path):
        raise UsageError("Cannot find clustering file: %s" % path)
    text = open(path).read()
    try:
        return [int(x) for x in text.split(",") if x.strip()]
    except ValueError:
        raise UsageError("Invalid string to split: %s" % text.strip()) from None


class Plan:
    """What the flags and the input names decide, before any data is read."""

    def __init__(self, flags: Flags):
        self.flags = flags
        validate(flags)
        self.chromosome_ids = [chromosome_to_id(c) for c in flags.chromosomes.split(",")]
        self.files = input_files(flags.i)
        if not self.files:
            return
        self.positions = read_positions(flags.pos_file) if flags.pos_file else []
        if flags.pos_file and len(self.positions) < len(self.files):
            raise UsageError("Number of chromosomes in %s (%d) does not match number of input files (%d)"
                             % (flags.pos_file, len(self.positions), len(self.files)))
        chrom = [get_chromosome(f) for f in self.files]
        for c in self.chromosome_ids:
            if c not in chrom:
                raise UsageError("Chromosome %s specified with --chromosomes=%s, but no input file for it was found"
                                 % (id_to_chromosome(c), flags.chromosomes))
        self.selected: List[Tuple[str, int]] = []
        seen: Dict[int, str] = {}
        for f, c in zip(self.files, chrom):
            if c not in self.chromosome_ids:
                continue
            if c in seen:
                raise UsageError("Two input files for chromosome %s: %s and %s" % (id_to_chromosome(c), seen[c], f))
            seen[c] = f
            self.selected.append((f, c))
        if flags.merge_file and not os.path.exists(flags.merge_file):
            raise UsageError("Cannot find merge file: " + flags.merge_file)
        self.clustering = read_clustering(flags.clustering) if flags.clustering else None

    def positions_of(self, chromosome_id: int) -> List[int]:
        return self.positions[chromosome_id] if chromosome_id < len(self.positions) else []


def _log(flags: Flags, msg: str) -> None:
    if flags.log_level not in ("warn", "warning", "err", "error", "critical", "off"):
        print(msg, flush=True)


def load(plan: Plan, sm_plan, id_to_group, times: dict):
    """-> (resident pileup, num_cells, max_read_length) over N_SLOTS chromosome slots."""
    import numpy as np

    from .pileup import FlatPileup
    from .pileup_load import read_pileups_resident
    from .pileup_reader import read_pileup

    f = plan.flags
    files = [p for p, _ in plan.selected]
    slots = [c for _, c in plan.selected]
    if all(p.endswith(".bin") for p in files):
        per: dict = {}
        res, num_cells, max_len = read_pileups_resident(
            sm_plan, files, slots, N_SLOTS, id_to_group, f.max_coverage,
            [plan.positions_of(c) for c in slots], f.compute_read_stats, times=times, per_file=per)
        if not files:
            num_cells, max_len = 0, 0
        return res, num_cells, max_len
    # text pileups (or a mix): the host reader per file, one upload
    parts = {}
    num_cells = max_len = 0
    for p, c in plan.selected:
        fp, nc, ml = read_pileup(p, id_to_group, None, f.max_coverage, plan.positions_of(c), f.compute_read_stats)
        parts[c] = fp
        num_cells, max_len = max(num_cells, nc), max(max_len, ml)
    chr_off = [0]
    pos, offs, rid, idb = [], [np.zeros(1, dtype=np.uint64)], [], []
    base = 0
    for c in range(N_SLOTS):
        fp = parts.get(c)
        if fp is not None:
            pos.append(fp.locus_pos)
            offs.append(np.asarray(fp.locus_entry_off[1:], dtype=np.uint64) + np.uint64(base))
            rid.append(fp.read_ids)
            idb.append(fp.id_base)
            base += fp.n_entries
        chr_off.append(chr_off[-1] + (fp.n_loci if fp is not None else 0))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)  # noqa: E731
    flat = FlatPileup(np.asarray(chr_off, dtype=np.uint32), cat(pos, np.uint32), cat(offs, np.uint64),
                      cat(rid, np.uint32), cat(idb, np.uint32))
    return sm_plan.upload(flat, None, max(int(np.max(id_to_group)) + 1, 1)), num_cells, max_len


def run(plan: Plan) -> int:
    import numpy as np

    from . import SimilarityMatrixPlan
    from .cluster import divide_cluster_resident
    from .pileup_reader import get_grouping
    from .variant import allele_stats, fasta_stats, tabix_stats, variant_calling_resident, vcf_stats

    f = plan.flags
    t0 = time.perf_counter()
    try:
        id_to_group = get_grouping(f.merge_count, f.merge_file, f.max_cell_count)
    except (FileNotFoundError, ValueError) as e:
        print(str(e), file=sys.stderr)
        return 1
    times = {}
    with SimilarityMatrixPlan(0) as sm:
        res, num_cells, max_read_length = load(plan, sm, id_to_group, times)
        t_load = time.perf_counter()
        _log(f, "Read %d loci, %d entries from %d files: %d cells, longest fragment %d"
             % (res["n_loci"], res["n_entries"], len(plan.selected), num_cells, max_read_length))
        if not f.merge_file:
            if len(id_to_group) < num_cells:
                print("--max_cell_count is %d, but number of cells is %d. Please add --max_cell_count=%d to the "
                      "command line" % (f.max_cell_count, num_cells, f.max_cell_count), file=sys.stderr)
                return 1
            id_to_group = id_to_group[:num_cells]
        elif num_cells != len(id_to_group):
            print("Invalid merge file %s. Merge files contains %d cell ids, data has %d cell ids"
                  % (f.merge_file, len(id_to_group), num_cells), file=sys.stderr)
            return 1
        num_groups = int(np.max(id_to_group)) + 1 if len(id_to_group) else 1
        ident = np.arange(num_groups, dtype=np.uint32)
        records = []
        if plan.clustering is None:
            clusters, _, records = divide_cluster_resident(
                sm, res, max_read_length, id_to_group, ident, ident, f.mutation_rate, f.homozygous_filtered_rate,
                f.seq_error_rate, f.normalization, f.termination, f.clustering_type, f.arma_kmeans,
                f.expectation_maximization, f.min_cluster_size, f.tumor_purity - 1, "", None, 1, with_times=True,
                out_dir=f.o)
        else:
            _log(f, "Using provided clustering file %s" % f.clustering)
            clusters = np.asarray(plan.clustering, dtype=np.uint16)
            if len(clusters) != num_cells:
                print("Number of clusters (%d) doesn't match number of cells (%d)" % (len(clusters), num_cells),
                      file=sys.stderr)
                return 1
        t_cluster = time.perf_counter()
        vc_times = None
        if f.reference_genome:
            _log(f, "Performing variant calling against %s" % f.reference_genome)
            vc_times = variant_calling_resident(sm, res, clusters, f.reference_genome, f.map_file, 1e-3,
                                                f.seq_error_rate, f.o, fasta_route=f.fasta_route or None,
                                                vcf_output=f.vcf_output or None, vcf_index=f.vcf_index or None,
                                                allele_counts=f.allele_counts or None,
                                                cell_names=f.cell_names or None)
            fs = fasta_stats()
            vc_times["fasta"] = "%s on %s" % (fs["kind"], fs["route"])
            if fs["route"] == "device":  # the device route's split; the three overlap
                vc_times.update(fasta_inflate_ms=fs["inflate_ms"], fasta_upload_ms=fs["upload_ms"],
                                fasta_parse_gather_ms=fs["parse_gather_ms"])
            vs = vcf_stats()
            vc_times["vcf"] = "%s, %d files, %d bytes of text" % (vs["output"], vs["files"], vs["text_bytes"])
            if vs["output"] == "bgzf":
                vc_times["vcf"] += ", %d compressed in %d blocks (%d stored)" % (
                    vs["compressed_bytes"], vs["blocks"], vs["stored_blocks"])
                vc_times.update(vcf_format_ms=vs["format_ms"], vcf_deflate_ms=vs["deflate_ms"],
                                vcf_download_ms=vs["download_ms"], vcf_write_ms=vs["write_ms"])
            ts = tabix_stats()
            if ts["files"]:
                vc_times["tbi"] = "%d files, %d data lines, %d chunks, %d bytes in %d" % (
                    ts["files"], ts["data_lines"], ts["chunks"], ts["index_bytes"], ts["compressed_bytes"])
                vc_times.update(tbi_pass_ms=ts["pass_ms"], tbi_build_ms=ts["build_ms"],
                                tbi_deflate_ms=ts["deflate_ms"], tbi_write_ms=ts["write_ms"])
            als = allele_stats()
            if als["selection"] != "none":
                vc_times["alleles"] = "%s, %d sites, %d pairs, %d bytes of text in %d ranges" % (
                    als["selection"], als["sites"], als["pairs"], als["text_bytes"], als["ranges"])
                vc_times.update(allele_count_ms=als["count_ms"], allele_format_ms=als["format_ms"],
                                allele_deflate_ms=als["deflate_ms"], allele_download_ms=als["download_ms"],
                                allele_write_ms=als["write_ms"])
        else:
            _log(f, "Skipping variant calling, because no reference genome was provided")
        t_end = time.perf_counter()
    for r in records:
        _log(f, "level %-6s cells %5d  kept loci %8d  coverage %8.3f  clusters %d  stop %s"
             % (repr(r["marker"]), r["cells"], r["kept_loci"], r["coverage"], r["num_clusters"], r["stop_reason"]))
    _log(f, "times: load %.1f ms (%s), clustering %.1f ms, variant calling %.1f ms%s, total %.1f ms" % (
        1e3 * (t_load - t0), ", ".join("%s %.1f" % kv for kv in times.items()) or "host reader",
        1e3 * (t_cluster - t_load), 1e3 * (t_end - t_cluster),
        "" if vc_times is None else " (%s)" % ", ".join(
            ("%s %.1f" if isinstance(kv[1], float) else "%s %s") % kv for kv in vc_times.items()),
        1e3 * (t_end - t0)))
    _log(f, "Done.")
    return 0


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    if not argv:
        print(usage())
        return 1
    try:
        flags = parse_flags(argv)
        plan = Plan(flags)
    except UsageError as e:
        print(str(e), file=sys.stderr)
        return 1
    if not plan.files:
        print("No input files found in %s. Nothing to do." % flags.i)
        return 0
    return run(plan)


if __name__ == "__main__":
    sys.exit(main())
