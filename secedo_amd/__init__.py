"""secedo_amd -- MI355X-native similarity-matrix path of SECEDO (computeSimilarityMatrix).

Only what the path needs: the HIP kernels + C-ABI (csrc/, include/secedo_simmat.h) and the
host-side mirror of the reference interface (similarity_matrix.py).
"""
from .pileup import FlatPileup, PosData, flatten  # noqa: F401
from .similarity_matrix import (InvalidNormalization, NORMALIZATIONS, PackingRoute, SecedoError,  # noqa: F401
                                SimilarityMatrixPlan, compute_similarity_matrix, get_devices, llr, llr_closed_form,
                                set_devices, to_enum)
from .filter import Filter, NO_POS, filter_resident  # noqa: F401,E402
from .pileup_reader import get_grouping, read_pileup  # noqa: F401,E402
from .spectral import laplacian, smallest_eigenpairs  # noqa: F401,E402
from .em import expectation_maximization  # noqa: F401,E402
from .cluster import divide_cluster, divide_cluster_resident, spectral_clustering  # noqa: F401,E402
from .variant import (allele_counts, allele_masks, allele_stats, bgzf_deflate, fasta_stats,  # noqa: F401,E402
                      genome_bins, genome_bins_stats, get_allele_counts, get_fasta_route, get_vcf_index,
                      get_vcf_output, reference_genotypes,
                      set_allele_counts, set_cell_names, set_fasta_route, set_vcf_index, set_vcf_output, tabix_build,
                      tabix_stats, variant_calling, variant_calling_resident, variant_calls, vcf_stats)
from .bam_pileup import (bam_barcodes, bam_index_build, bam_index_ranges, bam_index_stats, bam_route_stats,  # noqa: F401,E402
                         bam_scan, bam_select_stats, bgzf_inflate, bin_depth, depth_stats, pileup_bams,
                         pileup_bams_resident, set_index, split_clusters, split_rg_stats, split_select_stats,
                         split_stats)
from .sam_flags import FLAG_NAMES, parse_flags  # noqa: F401,E402
from .pileup_load import read_pileups_resident  # noqa: F401,E402
